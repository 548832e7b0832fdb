// aln_loop.hip -- device side of the heuristic loop's step (aln_pairset_loop_begin / aln_pairset_loop_step, include/aligner_hip.h): what
// stands between a held run of a pair set and the next run's going list.
//
//   classify   entry k of the held run (pair going[k]) against that pair's resident best f, by aln_loop_rules.h: finished (done or
//              failed) or improved; an improved pair's best becomes its f
//   settle     an improved entry's class once the transform kernel (aln_pairset.hip) has answered: going, or finished without a root
//   select     the entries of one kind -- improved, going, finished -- compacted in ascending entry order by a two-level prefix sum
//              (tile counts, one workgroup's scan over the tiles in trips of 256, tile-local scans): siblings of the three selection
//              kernels of aln_seqset.hip and aln_scan.hip, so that those stay as they are.  The same lists every run, no atomic appends.
//              improved: pair numbers and held entries (what the transform kernel reads); going: the next step's list of pair numbers
//              (what the pick kernel reads); finished: pair numbers, causes and the 48-byte summaries, packed for one download
//
// Every store is a plain C++ store of a thread (vector memory instructions); the prefix sums run in LDS.
#include <hip/hip_runtime.h>

#include "aln_device.h"
#include "aln_loop_rules.h"

#define LOOP_THREADS 256u
#define LOOP_PER_THREAD 8u
#define LOOP_TILE (LOOP_THREADS * LOOP_PER_THREAD)

// the kinds of a selection
#define LOOP_SEL_IMPROVED 0u
#define LOOP_SEL_GOING 1u
#define LOOP_SEL_FINISHED 2u

// ---- entry k of the held run: pair going[k], its summary res[k]
__global__ __launch_bounds__(256) void aln_loop_classify_kernel(const aln_pair_result *res, const uint32_t *going, uint32_t n, double *best,
                                                                uint32_t *cls)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t pair = going[k];
    const int32_t status = res[k].status;
    const double f = res[k].f;
    const uint32_t c = aln_loop_classify(status, f, best[pair]);
    if (c == ALN_LOOP_IMPROVED) best[pair] = f;          // a pair is listed once: no other thread reads or writes this word
    cls[k] = c;
}

// ---- listed transform c (held entry entry[c]; c itself without a table): going, or finished without a root
__global__ __launch_bounds__(256) void aln_loop_settle_kernel(const uint32_t *entry, const int32_t *transform_status, uint32_t n, uint32_t *cls)
{
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    cls[entry ? entry[c] : (uint32_t)c] = aln_loop_after_transform(transform_status[c]);
}

__device__ __forceinline__ bool loop_keep(uint32_t cls, uint32_t kind)
{
    return kind == LOOP_SEL_IMPROVED ? cls == ALN_LOOP_IMPROVED : kind == LOOP_SEL_GOING ? cls == ALN_LOOP_GOING : aln_loop_is_finished(cls);
}

// block-wide exclusive prefix sum of one value per thread (256 threads); returns the thread's offset, *total the block's sum
__device__ __forceinline__ uint32_t loop_block_scan(uint32_t v, uint32_t *lds, uint32_t *total)
{
    const uint32_t t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (uint32_t o = 1; o < LOOP_THREADS; o <<= 1) {
        const uint32_t add = t >= o ? lds[t - o] : 0u;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const uint32_t incl = lds[t];
    *total = lds[LOOP_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// ---- selection, step 1: kept entries per tile of LOOP_TILE entries (thread t looks at entries t*8 .. t*8+7 of the tile)
__global__ __launch_bounds__(256) void aln_loop_count_kernel(const uint32_t *cls, uint32_t n, uint32_t kind, uint32_t *tile_count)
{
    __shared__ uint32_t lds[LOOP_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * LOOP_TILE + (uint64_t)threadIdx.x * LOOP_PER_THREAD;
    uint32_t c = 0;
    for (uint32_t i = 0; i < LOOP_PER_THREAD; ++i)
        if (base + i < n && loop_keep(cls[base + i], kind)) ++c;
    uint32_t total;
    (void)loop_block_scan(c, lds, &total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// ---- selection, step 2: one workgroup turns the tile counts into tile offsets, 256 tiles a trip; count[0] = kept entries
__global__ __launch_bounds__(256) void aln_loop_offsets_kernel(const uint32_t *tile_count, uint32_t *tile_off, uint32_t tiles, uint32_t *count)
{
    __shared__ uint32_t lds[LOOP_THREADS];
    uint32_t carry = 0;
    for (uint32_t b = 0; b < tiles; b += LOOP_THREADS) {
        const uint32_t i = b + threadIdx.x;
        const uint32_t v = i < tiles ? tile_count[i] : 0u;
        uint32_t total;
        const uint32_t ex = loop_block_scan(v, lds, &total);
        if (i < tiles) tile_off[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) count[0] = carry;
}

// ---- selection, step 3: every tile writes its kept entries at its offset, in ascending order.  Kept entry k goes to place o:
// out_pair[o] = going[k] (k itself without a list); out_word[o] = k for the improved, the class (the cause) otherwise; out_res[o] =
// res[k] where asked for.  The outputs hold n entries: every entry may be kept.
__global__ __launch_bounds__(256) void aln_loop_compact_kernel(const uint32_t *cls, uint32_t n, uint32_t kind, const uint32_t *tile_off,
                                                               const uint32_t *going, const aln_pair_result *res, uint32_t *out_pair,
                                                               uint32_t *out_word, aln_pair_result *out_res)
{
    __shared__ uint32_t lds[LOOP_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * LOOP_TILE + (uint64_t)threadIdx.x * LOOP_PER_THREAD;
    uint32_t keep = 0, c = 0;
    for (uint32_t i = 0; i < LOOP_PER_THREAD; ++i)
        if (base + i < n && loop_keep(cls[base + i], kind)) { keep |= 1u << i; ++c; }
    uint32_t total;
    uint32_t o = tile_off[blockIdx.x] + loop_block_scan(c, lds, &total);
    for (uint32_t i = 0; i < LOOP_PER_THREAD; ++i)
        if (keep & (1u << i)) {
            const uint32_t k = (uint32_t)(base + i);
            if (o < n) {
                out_pair[o] = going ? going[k] : k;
                if (out_word) out_word[o] = kind == LOOP_SEL_IMPROVED ? k : cls[k];
                if (out_res) out_res[o] = res[k];
            }
            ++o;
        }
}

static inline uint32_t loop_blocks_of(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

extern "C" void aln_loop_launch_classify(const aln_pair_result *res, const uint32_t *going, uint32_t n, double *best, uint32_t *cls, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_loop_classify_kernel, dim3(loop_blocks_of(n, 256)), dim3(256), 0, s, res, going, n, best, cls);
}

extern "C" void aln_loop_launch_settle(const uint32_t *entry, const int32_t *transform_status, uint32_t n, uint32_t *cls, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(aln_loop_settle_kernel, dim3(loop_blocks_of(n, 256)), dim3(256), 0, s, entry, transform_status, n, cls);
}

extern "C" uint32_t aln_loop_tiles(uint32_t n) { return loop_blocks_of(n, LOOP_TILE); }

// tile_count / tile_off: aln_loop_tiles(n) words each; count[0]: the kept entries; kind: 0 improved, 1 going, 2 finished
extern "C" void aln_loop_launch_select(const uint32_t *cls, uint32_t n, uint32_t kind, const uint32_t *going, const aln_pair_result *res,
                                       uint32_t *tile_count, uint32_t *tile_off, uint32_t *count, uint32_t *out_pair, uint32_t *out_word,
                                       aln_pair_result *out_res, hipStream_t s)
{
    const uint32_t tiles = aln_loop_tiles(n);
    if (tiles) hipLaunchKernelGGL(aln_loop_count_kernel, dim3(tiles), dim3(LOOP_THREADS), 0, s, cls, n, kind, tile_count);
    hipLaunchKernelGGL(aln_loop_offsets_kernel, dim3(1), dim3(LOOP_THREADS), 0, s, tile_count, tile_off, tiles, count);
    if (tiles) hipLaunchKernelGGL(aln_loop_compact_kernel, dim3(tiles), dim3(LOOP_THREADS), 0, s, cls, n, kind, tile_off, going, res, out_pair,
                                  out_word, out_res);
}
