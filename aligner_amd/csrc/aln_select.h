// aln_select.h -- ordered compaction on the device, once: the two-level prefix sum behind the window selection (aln_scan.hip), the
// threshold selection of a sequence set (aln_seqset.hip), the three lists of the heuristic loop's step (aln_loop.hip) and the finish of
// the k best per row (aln_best.hip).
//
//   count      tile b = entries b * 2048 .. (thread t looks at entries t*8 .. t*8+7 of it): kept entries per tile -> tile_count[b]
//   offsets    one workgroup turns the tile counts into tile offsets, 256 tiles a trip; the sum of the trips before is the carry.
//              total[0] = kept entries in all
//   compact    every tile calls emit(o, k) for its kept entries k in ascending order, o = the entry's place among all kept entries
//
// Keep and Emit are small structs of device pointers and scalars, passed by value as kernel arguments: bool keep(uint64_t k),
// void emit(uint32_t o, uint64_t k).  emit checks o against the room of what it writes.  The same list every run, no atomic appends;
// every store is a plain C++ store of a thread (vector memory instructions), the prefix sums run in LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

constexpr uint32_t ALN_SELECT_THREADS = 256u;
constexpr uint32_t ALN_SELECT_PER_THREAD = 8u;
constexpr uint32_t ALN_SELECT_TILE = ALN_SELECT_THREADS * ALN_SELECT_PER_THREAD;

static inline uint64_t aln_select_tiles(uint64_t n) { return (n + ALN_SELECT_TILE - 1) / ALN_SELECT_TILE; }

// block-wide exclusive prefix sum of one value per thread (256 threads); returns the thread's offset, *total the block's sum
__device__ __forceinline__ uint32_t aln_block_exclusive_scan(uint32_t v, uint32_t *lds, uint32_t *total)
{
    const uint32_t t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (uint32_t o = 1; o < ALN_SELECT_THREADS; o <<= 1) {
        const uint32_t add = t >= o ? lds[t - o] : 0u;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const uint32_t incl = lds[t];
    *total = lds[ALN_SELECT_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// ---- step 1: kept entries per tile
template <class Keep>
__global__ __launch_bounds__(256) void aln_select_count_kernel(Keep keep, uint64_t n, uint32_t *tile_count)
{
    __shared__ uint32_t lds[ALN_SELECT_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * ALN_SELECT_TILE + (uint64_t)threadIdx.x * ALN_SELECT_PER_THREAD;
    uint32_t c = 0;
    for (uint32_t i = 0; i < ALN_SELECT_PER_THREAD; ++i)
        if (base + i < n && keep(base + i)) ++c;
    uint32_t total;
    (void)aln_block_exclusive_scan(c, lds, &total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// ---- step 2: tile counts -> tile offsets.  Off is uint32_t, or uint64_t where the kept entries of all tiles may pass 2^32 (the k best:
// 2^32 rows of 64).  The carry is an Off; a trip's sum stays in 32 bits (256 tile counts, of <= 2048 entries or <= 256 rows of 64 each)
template <class Off>
__global__ __launch_bounds__(256) void aln_select_offsets_kernel(const uint32_t *tile_count, Off *tile_off, uint64_t tiles, Off *total)
{
    __shared__ uint32_t lds[ALN_SELECT_THREADS];
    Off carry = 0;
    for (uint64_t b = 0; b < tiles; b += ALN_SELECT_THREADS) {
        const uint64_t i = b + threadIdx.x;
        const uint32_t v = i < tiles ? tile_count[i] : 0u;
        uint32_t trip;
        const uint32_t ex = aln_block_exclusive_scan(v, lds, &trip);
        if (i < tiles) tile_off[i] = carry + ex;
        carry += trip;
    }
    if (threadIdx.x == 0) total[0] = carry;
}

// ---- step 3: every tile hands its kept entries to emit at its offset, in ascending order (keep is evaluated once per entry)
template <class Keep, class Emit>
__global__ __launch_bounds__(256) void aln_select_compact_kernel(Keep keep, Emit emit, uint64_t n, const uint32_t *tile_off)
{
    __shared__ uint32_t lds[ALN_SELECT_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * ALN_SELECT_TILE + (uint64_t)threadIdx.x * ALN_SELECT_PER_THREAD;
    uint32_t kept = 0, c = 0;
    for (uint32_t i = 0; i < ALN_SELECT_PER_THREAD; ++i)
        if (base + i < n && keep(base + i)) { kept |= 1u << i; ++c; }
    uint32_t total;
    uint32_t o = tile_off[blockIdx.x] + aln_block_exclusive_scan(c, lds, &total);
    for (uint32_t i = 0; i < ALN_SELECT_PER_THREAD; ++i)
        if (kept & (1u << i)) {
            emit(o, base + i);
            ++o;
        }
}

// tile_count / tile_off: aln_select_tiles(n) words each; count[0]: the kept entries (written for n == 0 too)
template <class Keep, class Emit>
static inline void aln_select_launch(Keep keep, Emit emit, uint64_t n, uint32_t *tile_count, uint32_t *tile_off, uint32_t *count, hipStream_t s)
{
    const uint64_t tiles = aln_select_tiles(n);
    if (tiles) hipLaunchKernelGGL(aln_select_count_kernel<Keep>, dim3((uint32_t)tiles), dim3(ALN_SELECT_THREADS), 0, s, keep, n, tile_count);
    hipLaunchKernelGGL(aln_select_offsets_kernel<uint32_t>, dim3(1), dim3(ALN_SELECT_THREADS), 0, s, tile_count, tile_off, tiles, count);
    if (tiles) hipLaunchKernelGGL((aln_select_compact_kernel<Keep, Emit>), dim3((uint32_t)tiles), dim3(ALN_SELECT_THREADS), 0, s, keep, emit, n, tile_off);
}
