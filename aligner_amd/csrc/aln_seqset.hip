// aln_seqset.hip -- device side of the resident sequence set (aln_seqset_*, include/aligner_hip.h): the kernels that stand between
// S resident sequences and the existing fill / traceback machinery of aln_kernels.hip.
//
//   expand     pairs k0 .. k0 + n - 1 of a block of the S x S grid (aln_seqset_rules.h) -> PairDesc 0 .. n - 1 of a chunk (+ the queue
//              entries 0 .. n - 1): offsets and lengths out of the resident tables, built where they are used.  k is 64-bit (a block
//              may hold more than 2^32 pairs); descriptor and queue entry are chunk-local
//   gather     f and status of every pair of the chunk out of the 48-byte summaries (8 + 4 bytes per pair go back instead of 48), and
//              the first failed pair of the chunk as one word
//   select     status == ALN_OK and f >= f_min per pair, compacted in ascending pair order by the scan's two-level prefix sum (tile
//              counts, one workgroup's scan over the tiles, tile-local scans; aln_scan.hip has the same three steps for its z test --
//              a sibling, so that the scan's kernels stay as they are): the same list every run, no atomic appends
//   held       the listed held hits' summaries and both strings (aln_len bytes each), packed for one download
//
// Every store is a plain C++ store or an atomicMax of a thread (vector memory instructions).  The threshold test is a plain IEEE
// compare: a NaN f_min (or f) fails it.
#include <hip/hip_runtime.h>

#include "aln_device.h"
#include "aln_seqset_rules.h"

#define SEQSET_THREADS 256u
#define SEQSET_PER_THREAD 8u
#define SEQSET_TILE (SEQSET_THREADS * SEQSET_PER_THREAD)

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

// block-wide exclusive prefix sum of one value per thread (256 threads); returns the thread's offset, *total the block's sum
__device__ __forceinline__ uint32_t seqset_block_scan(uint32_t v, uint32_t *lds, uint32_t *total)
{
    const uint32_t t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (uint32_t o = 1; o < SEQSET_THREADS; o <<= 1) {
        const uint32_t add = t >= o ? lds[t - o] : 0u;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const uint32_t incl = lds[t];
    *total = lds[SEQSET_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// ---- selection, step 1: kept pairs per tile of SEQSET_TILE pairs (thread t looks at pairs t*8 .. t*8+7 of the tile)
__global__ __launch_bounds__(256) void aln_seqset_count_kernel(const aln_pair_result *res, uint64_t n, double f_min, uint32_t *tile_count)
{
    __shared__ uint32_t lds[SEQSET_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * SEQSET_TILE + (uint64_t)threadIdx.x * SEQSET_PER_THREAD;
    uint32_t c = 0;
    for (uint32_t i = 0; i < SEQSET_PER_THREAD; ++i)
        if (base + i < n && seqset_keep(res[base + i], f_min)) ++c;
    uint32_t total;
    (void)seqset_block_scan(c, lds, &total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// ---- selection, step 2: one workgroup turns the tile counts into tile offsets; count[0] = kept pairs of the chunk
__global__ __launch_bounds__(256) void aln_seqset_offsets_kernel(const uint32_t *tile_count, uint32_t *tile_off, uint64_t tiles, uint32_t *count)
{
    __shared__ uint32_t lds[SEQSET_THREADS];
    uint32_t carry = 0;
    for (uint64_t b = 0; b < tiles; b += SEQSET_THREADS) {
        const uint64_t i = b + threadIdx.x;
        const uint32_t v = i < tiles ? tile_count[i] : 0u;
        uint32_t total;
        const uint32_t ex = seqset_block_scan(v, lds, &total);
        if (i < tiles) tile_off[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) count[0] = carry;
}

// ---- selection, step 3: every tile writes its kept pairs at its offset, in ascending order: the pair's number in the block and its f
// (hit_k / hit_f hold n entries: every pair may pass)
__global__ __launch_bounds__(256) void aln_seqset_compact_kernel(const aln_pair_result *res, uint64_t n, uint64_t k0, double f_min,
                                                                 const uint32_t *tile_off, uint64_t *hit_k, double *hit_f)
{
    __shared__ uint32_t lds[SEQSET_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * SEQSET_TILE + (uint64_t)threadIdx.x * SEQSET_PER_THREAD;
    uint32_t keep = 0, c = 0;
    for (uint32_t i = 0; i < SEQSET_PER_THREAD; ++i)
        if (base + i < n && seqset_keep(res[base + i], f_min)) { keep |= 1u << i; ++c; }
    uint32_t total;
    uint32_t o = tile_off[blockIdx.x] + seqset_block_scan(c, lds, &total);
    for (uint32_t i = 0; i < SEQSET_PER_THREAD; ++i)
        if (keep & (1u << i)) {
            if (o < n) { hit_k[o] = k0 + base + i; hit_f[o] = res[base + i].f; }
            ++o;
        }
}

// ---- held hits: listed entry k = held hit list[k]: its summary, and both strings at out_tb + out_off[k] (query, then target cap
// bytes later)
__global__ __launch_bounds__(256) void aln_seqset_held_kernel(const PairsetHeld *held, const aln_pair_result *res, const uint8_t *tb,
                                                              const uint32_t *list, const uint64_t *out_off, uint32_t n_held,
                                                              aln_pair_result *out_res, uint8_t *out_tb)
{
    const uint32_t k = blockIdx.x, h = list[k];
    if (h >= n_held) return;                                         // checked on the host; never read beyond the held hits
    const aln_pair_result r = res[h];
    if (threadIdx.x == 0) out_res[k] = r;
    if (r.status != ALN_OK || !out_tb) return;
    const PairsetHeld d = held[h];
    const uint32_t cap = d.N + d.M + 2u;
    const uint32_t len = r.aln_len < cap ? r.aln_len : cap;
    const uint8_t *__restrict__ src = tb + d.tb_off;
    uint8_t *__restrict__ dst = out_tb + out_off[k];
    for (uint32_t j = threadIdx.x; j < len; j += blockDim.x) { dst[j] = src[j]; dst[cap + j] = src[cap + j]; }
}

static inline uint32_t blocks_of(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

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

extern "C" uint64_t aln_seqset_tiles(uint64_t n) { return (n + SEQSET_TILE - 1) / SEQSET_TILE; }

// tile_count / tile_off: aln_seqset_tiles(n) words each; hit_k / hit_f: n entries each; count[0]: the chunk's hits
extern "C" void aln_seqset_launch_select(const aln_pair_result *res, uint64_t n, uint64_t k0, double f_min, uint32_t *tile_count,
                                         uint32_t *tile_off, uint32_t *count, uint64_t *hit_k, double *hit_f, hipStream_t s)
{
    const uint64_t tiles = aln_seqset_tiles(n);
    if (tiles) hipLaunchKernelGGL(aln_seqset_count_kernel, dim3((uint32_t)tiles), dim3(SEQSET_THREADS), 0, s, res, n, f_min, tile_count);
    hipLaunchKernelGGL(aln_seqset_offsets_kernel, dim3(1), dim3(SEQSET_THREADS), 0, s, tile_count, tile_off, tiles, count);
    if (tiles) hipLaunchKernelGGL(aln_seqset_compact_kernel, dim3((uint32_t)tiles), dim3(SEQSET_THREADS), 0, s, res, n, k0, f_min, tile_off,
                                  hit_k, hit_f);
}

extern "C" void aln_seqset_launch_held(const PairsetHeld *held, const aln_pair_result *res, const uint8_t *tb, const uint32_t *list,
                                       const uint64_t *out_off, uint32_t n_list, uint32_t n_held, aln_pair_result *out_res, uint8_t *out_tb,
                                       hipStream_t s)
{
    if (n_list) hipLaunchKernelGGL(aln_seqset_held_kernel, dim3(n_list), dim3(256), 0, s, held, res, tb, list, out_off, n_held, out_res, out_tb);
}
